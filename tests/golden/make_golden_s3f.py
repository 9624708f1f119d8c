"""Records tests/golden/S3F_toy/: the toy assays of the S3F CLI test, a synthetic surface file in the reference's format, and the
outputs of the reference's own SurfGVP.

    python tests/golden/make_golden_s3f.py --reference <ProteinGym checkout>

The reference's s3f/gvp_layer.py and s3f/gvp.py are imported unmodified and run on the CPU in float64, over the stand-ins of
make_golden_s2f.py plus three of this file's for what SurfGVP alone touches:
  * ``torch_cluster.knn_graph(pos, k, batch)``: per graph of the batch, every point's k nearest other points; edge_index row 0 = the
    neighbour (source), row 1 = the centre (target), no self loops;
  * ``s3f.surface.knn_atoms(x, y, k, batch_x, batch_y)``: per graph, the k + 1 nearest rows of y for each row of x by squared
    distance, nearest first, as global row indices, and those squared distances (pykeops' argKmin under block-diagonal ranges);
  * the graph attributes SurfGVP.forward reads: edge_list, node_position, res2surf, residue2graph, node2graph on the residue graph;
    node_position, node_feature, node2graph, num_node, num_nodes, num_cum_nodes on the packed surface graph.
What they encode is the libraries' documented behaviour, not something run here: DESIGN.md 4.6p lists it.  The surface file is
synthetic (seeded points around the toy backbone, seeded features, res2surf by brute force); producing real ones is
script/process_surface.py's.  No test imports this file; only the files it writes are committed."""
import argparse
import os
import pickle
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
OUT = os.path.join(HERE, "S3F_toy")
L_TOY, L_CUT, D_TOY, NS_TOY = 37, 30, 128, 250


def knn_graph(pos, k, batch=None):
    batch = torch.zeros(len(pos), dtype=torch.int64) if batch is None else batch
    d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1)
    d2 = d2.masked_fill(batch[:, None] != batch[None, :], float("inf"))
    d2.fill_diagonal_(float("inf"))
    nb = d2.argsort(dim=1, stable=True)[:, :k]
    return torch.stack([nb.reshape(-1), torch.arange(len(pos)).repeat_interleave(k)])


def knn_atoms(x, y, k, batch_x=None, batch_y=None):
    k = k + 1
    d2 = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    if batch_x is not None:
        d2 = d2.masked_fill(batch_x[:, None] != batch_y[None, :], float("inf"))
    idx = d2.argsort(dim=1, stable=True)[:, :k]
    return idx, ((x[:, None, :] - y[idx]) ** 2).sum(-1)


def toy_files():
    import s2f_cases
    import s3f_cases
    import s3f_ref
    from proteingym_amd import s2f
    pos, plddt = s2f_cases.toy(L_TOY)
    rng = np.random.default_rng(43)
    seq = "".join(rng.choice(list(s2f.RESIDUE_ORDER), L_TOY))
    three = dict(zip("GASPVTCILNDQKEMHFRYW", "GLY ALA SER PRO VAL THR CYS ILE LEU ASN ASP GLN LYS GLU MET HIS PHE ARG TYR TRP".split()))
    os.makedirs(os.path.join(OUT, "EVE"), exist_ok=True)
    atoms = (("N", -1.2), ("CA", 0.0), ("C", 1.3))
    with open(os.path.join(OUT, "toy.pdb"), "w") as f:
        for i, (a, p, b) in enumerate(zip(seq, pos, plddt)):
            for n, (name, d) in enumerate(atoms):
                f.write("ATOM  %5d  %-3s %3s A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f           %s\n" %
                        (3 * i + n + 1, name, three[a], i + 1, p[0] + d, p[1], p[2], 1.0, b if name == "CA" else 1.0, name[0]))
        f.write("END\n")
    # the surface: the k-NN lists must be unambiguous on the whole cloud and on the cloud the 30-residue window keeps
    ca = s2f.read_ca(os.path.join(OUT, "toy.pdb"))[0]
    for seed in range(100):
        pts, feat = s3f_cases.make(ca, NS_TOY, 7000 + seed)
        xyz = np.stack([ca.astype(np.float64) + np.array([d, 0.0, 0.0]) for _, d in atoms], 1)          # [L, 3 atoms, 3]
        r2s = s3f_ref.nearest(xyz.reshape(-1, 3), pts, 21)[0].reshape(L_TOY, 3, 21).astype(np.int64)
        kept = s3f_ref.truncate(pts, feat, r2s, 0, 0, L_CUT)[0]
        if len(kept) < NS_TOY and min(s3f_cases.margins(ca[:L_CUT], kept)) > s3f_cases.MARGIN and \
                min(s3f_cases.margins(ca, s3f_ref.truncate(pts, feat, r2s, 0, 0, L_TOY)[0])) > s3f_cases.MARGIN:
            break
    else:
        raise RuntimeError("no seed gives unambiguous k-NN lists")
    nrm = rng.standard_normal((NS_TOY, 3)).astype(np.float32)
    with open(os.path.join(OUT, "toy.pkl"), "wb") as f:
        pickle.dump(dict(surf_points=pts, surf_normals=nrm / np.linalg.norm(nrm, axis=1, keepdims=True), surf_hks=feat[:, :32].copy(),
                         surf_curvatures=feat[:, 32:].copy(), res2surf=r2s), f, protocol=4)
    with open(os.path.join(OUT, "reference.csv"), "w") as f:
        f.write("DMS_index,DMS_id,DMS_filename,target_seq,seq_len,DMS_number_single_mutants,pdb_file,pdb_range\n")
        f.write(f"0,TOY_S3F,TOY_S3F.csv,{seq},{L_TOY},6,toy.pdb,1-{L_TOY}\n")
        f.write(f"1,TOY_S3F_CUT,TOY_S3F_CUT.csv,{seq[:L_CUT]},{L_CUT},5,toy.pdb,1-{L_TOY}\n")       # the structure is longer than the window
    for name, L, n_single, n_all in (("TOY_S3F", L_TOY, 6, 11), ("TOY_S3F_CUT", L_CUT, 5, 8)):
        muts = set()
        while len(muts) < n_all:
            k = 1 if len(muts) < n_single else 2
            ps = sorted(int(p) for p in rng.choice(L - 1, k, replace=False))
            muts.add(":".join(seq[p] + str(p + 1) + str(rng.choice([a for a in s2f.RESIDUE_ORDER if a != seq[p]])) for p in ps))
        first = sorted(m for m in muts if ":" not in m)[0]          # a second mutant at a site set already there: one masked sequence, two rows
        muts.add(first[:-1] + [a for a in s2f.RESIDUE_ORDER if a not in (first[0], first[-1])][0])
        muts = list(rng.permutation(sorted(muts)))
        with open(os.path.join(OUT, name + ".csv"), "w") as f:
            f.write("mutant,mutated_sequence,DMS_score,DMS_score_bin\n")
            for m in muts:
                s = list(seq[:L])
                for sub in m.split(":"):
                    s[int(sub[1:-1]) - 1] = sub[-1]
                f.write(f"{m},{''.join(s)},{rng.standard_normal():.4f},1\n")
        with open(os.path.join(OUT, "EVE", name + ".csv"), "w") as f:     # another order, three mutants missing, one never assayed
            f.write("mutant,EVE_ensemble\n")
            for m in list(rng.permutation(muts[:-3])) + ["A1C"]:
                f.write(f"{m},{rng.standard_normal():.5f}\n")
    with open(os.path.join(OUT, "s3f_toy.yaml"), "w") as f:
        f.write("summary:\n  class: ProteinGym\n  path: {{ datadir }}\n  csv_file: reference.csv\n\nstructure_path: {{ structdir }}\n"
                "surface_path: {{ surfdir }}\n\ntask:\n  class: ResidueTypePrediction\n  mask_rate: 0.15\n  dropout: 0.5\n"
                "  plddt_threshold: 70\n  model:\n    class: FusionNetwork\n    sequence_model:\n      class: MyESM\n      model: toy\n"
                f"    structure_model:\n      class: SurfGVP\n      node_in_dim: [{D_TOY}, 0]\n      node_h_dim: [256, 16]\n"
                "      edge_in_dim: [16, 1]\n      edge_h_dim: [64, 1]\n      surf_in_dim: [42, 0]\n      surf_edge_in_dim: [16, 1]\n"
                "      num_surf_res_neighbor: 3\n      num_surf_graph_neighbor: 16\n      num_layers: 5\n      vector_gate: True\n"
                "      readout: mean\n      drop_rate: 0.1\n  graph_construction_model:\n    class: GraphConstruction\n    node_layers:\n"
                "      - class: AlphaCarbonNode\n    edge_layers:\n      - class: SpatialEdge\n        radius: 10.0\n        min_distance: 0\n"
                "    edge_feature: null\n\ngpus: [0]\nbatch_size: 2\n\nmodel_checkpoint: {{ ckpt }}\n")


def packed(pos, edges, r2s, spos, feat, copies):
    """The residue graph and the surface graph of `copies` copies of one structure, as a torchdrug loader packs them."""
    L, ns = len(pos), len(spos)
    e = torch.cat([edges + b * L for b in range(copies)], 1)
    graph = types.SimpleNamespace(edge_list=torch.cat([e.t(), torch.zeros(e.shape[1], 1, dtype=torch.int64)], 1),
                                  node_position=torch.as_tensor(np.array(pos)).double().repeat(copies, 1),
                                  res2surf=torch.as_tensor(r2s).repeat(copies, 1, 1),
                                  residue2graph=torch.arange(copies).repeat_interleave(L), node2graph=torch.arange(copies).repeat_interleave(L))
    surf = types.SimpleNamespace(node_position=torch.as_tensor(np.array(spos)).double().repeat(copies, 1),
                                 node_feature=torch.as_tensor(np.array(feat)).double().repeat(copies, 1),
                                 node2graph=torch.arange(copies).repeat_interleave(ns), num_node=copies * ns,
                                 num_nodes=torch.full((copies,), ns), num_cum_nodes=torch.arange(1, copies + 1) * ns)
    return graph, surf


def record(reference):
    import make_golden_s2f
    import s2f_cases
    import s2f_ref
    import s3f_ref
    from proteingym_amd import s2f, s3f, synthetic
    make_golden_s2f.install_stand_ins()
    sys.modules["torch_cluster"].knn_graph = knn_graph
    sys.modules["s3f.surface"].knn_atoms = knn_atoms
    sys.path.insert(0, os.path.join(reference, "proteingym", "baselines", "S3F"))
    from s3f import gvp
    esm_cfg = dict(synthetic.ESM2_650M, layers=2, embed_dim=D_TOY, heads=2, ffn_dim=256)
    sd = s3f.random_state_dict(5, esm_cfg)
    net = gvp.SurfGVP(node_in_dim=(D_TOY, 0), node_h_dim=(256, 16), edge_in_dim=(16, 1), edge_h_dim=(64, 1), surf_in_dim=(42, 0),
                      surf_edge_in_dim=(16, 1), num_surf_graph_neighbor=16, num_surf_res_neighbor=3, readout="mean", num_layers=5,
                      drop_rate=0.1, vector_gate=True).double().eval()
    own = {k[len(s2f_ref.SM):]: torch.as_tensor(v).double() for k, v in sd.items() if k.startswith(s2f_ref.SM)}
    res = net.load_state_dict(own, strict=False)
    assert not res.unexpected_keys and all(k.endswith("dummy_param") for k in res.missing_keys), res
    pos, _ = s2f.read_ca(os.path.join(OUT, "toy.pdb"))
    with open(os.path.join(OUT, "toy.pkl"), "rb") as f:
        d = pickle.load(f)
    spos, feat, r2s = s3f_ref.read_surfaces([d])
    x = torch.as_tensor(s2f_cases.inputs(L_TOY, 2, D_TOY)[0]).double()
    edges = s2f_ref.radius_edges(pos)
    with torch.no_grad():
        g1, s1 = packed(pos, edges, r2s, spos, feat, 1)
        none = net.residue2surface(g1, s1) is None                  # the method has no return: forward indexes with None
        out1 = net(g1, x[0], s1)["node_feature"]
        g2, s2 = packed(pos, edges, r2s, spos, feat, 2)
        out2 = net(g2, x.reshape(-1, D_TOY), s2)["node_feature"]
        ei, h0, (rbf, vec) = net.surface_feature_init(g1, s1, x[0])
        hs = net.surf_W_v(h0)
        he = net.surf_W_e((rbf, vec))
        l0s, l0v = net.surf_layers[0](hs, ei, he)
        h = hs
        for layer in net.surf_layers:
            h = layer(h, ei, he)
        pooled = net.surf_W_out(h)[None].mean(dim=1)
    assert none and out1.shape == (L_TOY, 256) and out2.shape == (2 * L_TOY, 256) and pooled.shape == (1, 256)
    np.savez_compressed(os.path.join(OUT, "reference_modules.npz"), residue2surface_is_none=np.array(none), node_feature_1=out1.numpy(),
                        node_feature_2=out2.numpy(), init_edge_index=ei.numpy(), init_node=h0[:96].numpy(), init_rbf=rbf[:320].numpy(),
                        init_vec=vec[:, 0].numpy(), layer0_s=l0s[:96].numpy(), layer0_v=l0v.numpy(), pooled=pooled[0].numpy())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a ProteinGym checkout (proteingym/baselines/S3F is read)")
    args = ap.parse_args()
    toy_files()
    record(args.reference)
