"""Records tests/golden/S2F_toy/: the toy assay of the S2F CLI test and the outputs of the reference's own GVP modules.

    python tests/golden/make_golden_s2f.py --reference <ProteinGym checkout>

The reference's s3f/gvp_layer.py and s3f/gvp.py are imported unmodified and run on the CPU in float64.  The libraries they import are
not installed, so this script supplies small stand-ins for exactly what those two files use: a ``MessagePassing`` whose propagate
gathers (x_j, x_i) by edge_index = (source j, target i) and averages the messages at i, ``scatter_add``, torchdrug's registry
decorator, ``Configurable``, the readouts, the ``device`` property torchdrug patches onto nn.Module, and empty ``knn_graph`` /
``s3f.surface`` modules.  What the stand-ins encode (flow direction, mean over incoming edges) is the libraries' documented
behaviour, not something run here: DESIGN.md 4.6n lists it.  No test imports this file; only the arrays and the toy assay it writes
are committed."""
import argparse
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(HERE, "S2F_toy")
L_TOY, D_TOY = 37, 128


def install_stand_ins():
    class MessagePassing(nn.Module):
        def __init__(self, aggr="mean"):
            super().__init__()
            self.aggr = aggr

        def propagate(self, edge_index, s, v, edge_attr):
            j, i = edge_index
            msg = self.message(s_i=s[i], v_i=v[i], s_j=s[j], v_j=v[j], edge_attr=edge_attr)
            out = torch.zeros(s.shape[0], msg.shape[1], dtype=msg.dtype).index_add_(0, i, msg)
            if self.aggr == "mean":
                cnt = torch.zeros(s.shape[0], dtype=msg.dtype).index_add_(0, i, torch.ones(len(i), dtype=msg.dtype))
                out = out / cnt.clamp(min=1)[:, None]
            return out

    def scatter_add(src, index, dim=0, dim_size=None):
        return torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, src)

    class Registry:
        @staticmethod
        def register(name):
            return lambda cls: cls

    class Readout(nn.Module):
        def forward(self, graph, x):
            return x.mean(0, keepdim=True)

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    core = module("torchdrug.core", Configurable=type("Configurable", (), {}), Registry=Registry)
    layers = module("torchdrug.layers", SumReadout=Readout, MeanReadout=Readout)
    module("torchdrug", core=core, layers=layers)
    tg_nn = module("torch_geometric.nn", MessagePassing=MessagePassing)
    module("torch_geometric", nn=tg_nn)
    module("torch_scatter", scatter_add=scatter_add)
    module("torch_cluster", knn_graph=None)
    module("s3f.surface")
    nn.Module.device = property(lambda self: next(self.parameters()).device)


def toy_assay():
    import s2f_cases
    from proteingym_amd import s2f
    pos, plddt = s2f_cases.toy(L_TOY)
    rng = np.random.default_rng(41)
    seq = "".join(rng.choice(list(s2f.RESIDUE_ORDER), L_TOY))
    muts = set()
    while len(muts) < 14:
        k = 1 if len(muts) < 8 else 2
        ps = sorted(int(p) for p in rng.choice(L_TOY - 1, k, replace=False))
        muts.add(":".join(seq[p] + str(p + 1) + str(rng.choice([a for a in s2f.RESIDUE_ORDER if a != seq[p]])) for p in ps))
    muts = list(rng.permutation(sorted(muts)))
    three = dict(zip("GASPVTCILNDQKEMHFRYW", "GLY ALA SER PRO VAL THR CYS ILE LEU ASN ASP GLN LYS GLU MET HIS PHE ARG TYR TRP".split()))
    os.makedirs(os.path.join(OUT, "EVE"), exist_ok=True)
    with open(os.path.join(OUT, "toy.pdb"), "w") as f:
        for i, (a, p, b) in enumerate(zip(seq, pos, plddt)):
            for n, (name, d) in enumerate((("N", -1.2), ("CA", 0.0), ("C", 1.3))):       # N and C only so that the reader has to pick CA
                f.write("ATOM  %5d  %-3s %3s A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f           %s\n" %
                        (3 * i + n + 1, name, three[a], i + 1, p[0] + d, p[1], p[2], 1.0, b if name == "CA" else 1.0, name[0]))
        f.write("END\n")
    with open(os.path.join(OUT, "TOY_S2F.csv"), "w") as f:
        f.write("mutant,mutated_sequence,DMS_score,DMS_score_bin\n")
        for m in muts:
            s = list(seq)
            for sub in m.split(":"):
                s[int(sub[1:-1]) - 1] = sub[-1]
            f.write(f"{m},{''.join(s)},{rng.standard_normal():.4f},1\n")
    with open(os.path.join(OUT, "reference.csv"), "w") as f:
        f.write("DMS_index,DMS_id,DMS_filename,target_seq,seq_len,DMS_number_single_mutants,pdb_file,pdb_range\n")
        f.write(f"0,TOY_S2F,TOY_S2F.csv,{seq},{L_TOY},8,toy.pdb,1-{L_TOY}\n")
    with open(os.path.join(OUT, "EVE", "TOY_S2F.csv"), "w") as f:       # another order, three mutants missing, one never assayed
        f.write("mutant,EVE_ensemble\n")
        for m in list(rng.permutation(muts[:-3])) + ["A1C"]:
            f.write(f"{m},{rng.standard_normal():.5f}\n")
    with open(os.path.join(OUT, "s2f_toy.yaml"), "w") as f:
        f.write("summary:\n  class: ProteinGym\n  path: {{ datadir }}\n  csv_file: reference.csv\n\nstructure_path: {{ structdir }}\n"
                "surface_path: {{ surfdir }}\n\ntask:\n  class: ResidueTypePrediction\n  mask_rate: 0.15\n  dropout: 0.5\n"
                "  plddt_threshold: 70\n  model:\n    class: FusionNetwork\n    sequence_model:\n      class: MyESM\n      model: toy\n"
                f"    structure_model:\n      class: GVPGNN\n      node_in_dim: [{D_TOY}, 0]\n      node_h_dim: [256, 16]\n"
                "      edge_in_dim: [16, 1]\n      edge_h_dim: [64, 1]\n      num_layers: 5\n      vector_gate: True\n      readout: mean\n"
                "      drop_rate: 0.1\n  graph_construction_model:\n    class: GraphConstruction\n    node_layers:\n      - class: AlphaCarbonNode\n"
                "    edge_layers:\n      - class: SpatialEdge\n        radius: 10.0\n        min_distance: 0\n    edge_feature: null\n\n"
                "gpus: [0]\nbatch_size: 4\n\nmodel_checkpoint: {{ ckpt }}\n")


def record(reference):
    import s2f_cases
    import s2f_ref
    from proteingym_amd import s2f, synthetic
    install_stand_ins()
    sys.path.insert(0, os.path.join(reference, "proteingym", "baselines", "S3F"))
    from s3f import gvp, gvp_layer
    esm_cfg = dict(synthetic.ESM2_650M, layers=2, embed_dim=D_TOY, heads=2, ffn_dim=256)
    sd = s2f.random_state_dict(5, esm_cfg)
    net = gvp.GVPGNN(node_in_dim=(D_TOY, 0), node_h_dim=(256, 16), edge_in_dim=(16, 1), edge_h_dim=(64, 1), readout="mean", num_layers=5,
                     drop_rate=0.1, vector_gate=True).double().eval()
    own = {k[len(s2f_ref.SM):]: torch.as_tensor(v).double() for k, v in sd.items() if k.startswith(s2f_ref.SM)}
    res = net.load_state_dict(own, strict=False)
    assert not res.unexpected_keys and all(k.endswith("dummy_param") for k in res.missing_keys), res
    pos, _ = s2f_cases.toy(L_TOY)
    x = torch.as_tensor(s2f_cases.inputs(L_TOY, 1, D_TOY)[0][0]).double()
    edges = s2f_ref.radius_edges(pos)                       # the graph is an input here: torch_cluster is not run
    graph = types.SimpleNamespace(edge_list=torch.cat([edges.t(), torch.zeros(edges.shape[1], 1, dtype=torch.int64)], 1),
                                  node_position=torch.as_tensor(np.array(pos)).double())
    rng = np.random.default_rng(9)
    ts = torch.as_tensor(rng.standard_normal((11, 256)))
    tv = torch.as_tensor(rng.standard_normal((11, 16, 3)))
    tv[3] = 0.0                                             # a zero vector row: the clamps
    ms, mv = torch.as_tensor(rng.standard_normal((11, 576))), torch.as_tensor(rng.standard_normal((11, 33, 3)))
    with torch.no_grad():
        out = net(graph, x)["node_feature"]
        node_in, node_out = graph.edge_list.t()[:2]
        vec = graph.node_position[node_out] - graph.node_position[node_in]
        es, ev = net.W_e((gvp.rbf(vec.norm(dim=-1), dim=16), vec.unsqueeze(-2)))
        s0, v0 = net.W_v(net.residue_embdding(x))
        s1, v1 = net.layers[0]((s0, v0), graph.edge_list.t()[:2], (es, ev))
        gs, gv = net.layers[0].conv.message_func[0]((ms, mv))
        ls, lv = net.layers[0].norm[0]((ts, tv))
        fs, fv = net.layers[0].ff_func((ts, tv))
    np.savez_compressed(os.path.join(OUT, "reference_modules.npz"), edges=edges.numpy(), gnn_out=out.numpy(), edge_s=es[:160].numpy(),
                        edge_v=ev.numpy(), layer0_s=s1.numpy(), layer0_v=v1.numpy(), tuple_s=ts.numpy(), tuple_v=tv.numpy(),
                        msg_in_s=ms.numpy(), msg_in_v=mv.numpy(), gvp_s=gs.numpy(), gvp_v=gv.numpy(), ln_s=ls.numpy(), ln_v=lv.numpy(),
                        ff_s=fs.numpy(), ff_v=fv.numpy())
    assert gvp_layer.GVPConv.__mro__[1].__name__ == "MessagePassing"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a ProteinGym checkout (proteingym/baselines/S3F is read)")
    args = ap.parse_args()
    toy_assay()
    record(args.reference)
