"""Writes tests/golden/golden_esmif1.npz, esmif1_state_dict_keys.json (key names and shapes, and the reference parser's option strings), ESMIF1_structures/toy_esmif1.pdb and the TOY_ESMIF1* CSVs from
the UNMODIFIED reference ESM-IF1 (proteingym/baselines/esm: compute_fitness_esm_if1.py, esm/inverse_folding/*, esm/pretrained.py) on the
CPU.

    python tests/golden/make_golden_esmif1.py

It is run by hand where the reference tree is available and is not run by the tests.  Weights are tests/esmif1_cases.py's seeded toy
state dict and the backbones its seeded random walks: the tests rebuild both, so no checkpoint is committed.

Two packages the reference imports are not installed here and are stubbed in sys.modules before the import:
  biotite.*          empty stubs: only util.py's load_structure / extract_coords_from_structure use them, and they are not called.
  torch_geometric.nn a MessagePassing stand-in of a dozen lines with the default flow of the real one: `_j` arguments gathered at
                     edge_index[0], `_i` arguments at edge_index[1], message() called on them, and the messages averaged per
                     edge_index[1] (index_add, the count clamped to 1, so a node without incoming edges gets zeros).
Because biotite is missing, the reference's own PDB reading (util.py load_coords) has no executable oracle here.  For the toy assay the
attribute esm.inverse_folding.util.load_coords is replaced by proteingym_amd.esmif1.read_backbone on the committed toy PDB; everything
else of compute_fitness_esm_if1.score_singlechain_backbone_batch runs unmodified (nogpu=True).

float64: torch.set_default_dtype(torch.float64) and model.double(), coordinates as float64.  The places where the reference names float32
itself (the sinusoidal position tables, the edges' relative-position frequencies) stay float32 in that run, as they would in any float64
run of it.

What the file holds per case of esmif1_cases.CASES (backbone, two sequences): enc32 / enc64 = encoder_out [S, D]; lp32_i / lp64_i =
log_softmax of the logits [T_i, V] of sequence i; ll32 / ll64 = the scores (-mean cross-entropy).  All arrays float64 (the float32 run's
numbers widened).
"""
import importlib.machinery
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.ref_harness import REF_ROOT as REFERENCE  # noqa: E402

import esmif1_cases as K  # noqa: E402
from proteingym_amd import esmif1 as E  # noqa: E402


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        v = type(attr, (), {})
        setattr(self, attr, v)
        return v


class _StubFinder:
    def find_spec(self, name, path=None, target=None):
        return importlib.machinery.ModuleSpec(name, self) if name.split(".")[0] == "biotite" else None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def message_passing_stand_in():
    import torch

    class MessagePassing(torch.nn.Module):
        def __init__(self, aggr="mean"):
            super().__init__()
            assert aggr == "mean"

        def propagate(self, edge_index, s, v, edge_attr):
            j, i = edge_index[0], edge_index[1]
            msg = self.message(s_i=s[i], v_i=v[i], s_j=s[j], v_j=v[j], edge_attr=edge_attr)
            n = s.shape[0]
            total = torch.zeros(n, msg.shape[1], dtype=msg.dtype).index_add_(0, i, msg)
            count = torch.zeros(n, dtype=msg.dtype).index_add_(0, i, torch.ones(i.shape[0], dtype=msg.dtype))
            return total / count.clamp(min=1).unsqueeze(-1)
    return MessagePassing


def reference():
    sys.meta_path.insert(0, _StubFinder())
    tg, tgnn = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.nn")
    tgnn.MessagePassing = message_passing_stand_in()
    tg.nn = tgnn
    sys.modules["torch_geometric"], sys.modules["torch_geometric.nn"] = tg, tgnn
    for p in (REFERENCE, os.path.join(REFERENCE, "proteingym"), os.path.join(REFERENCE, "proteingym", "baselines", "esm")):
        sys.path.insert(0, p)
    import compute_fitness_esm_if1 as cf
    return cf


def build_model(cf, dtype):
    import torch
    esm = cf.esm
    alphabet = esm.data.Alphabet.from_architecture(K.TOY_ARGS["arch"])
    model = esm.inverse_folding.gvp_transformer.GVPTransformerModel(K.toy_args(), alphabet)
    cfg = E.config_from_args(K.toy_args())
    sd = {k: torch.from_numpy(v) for k, v in K.state_dict(cfg).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("_float_tensor") for k in missing), (missing, unexpected)
    return model.to(dtype).eval(), alphabet


def run_case(cf, model, alphabet, coords, seqs, dtype):
    import torch
    conv = cf.CoordBatchConverter(alphabet)
    enc, lps, lls = None, [], []
    for seq in seqs:
        c, conf, _, tokens, pad = conv([(coords.astype(np.float64 if dtype == torch.float64 else np.float32), None, seq)])
        with torch.no_grad():
            enc_out = model.encoder(c, pad, conf)["encoder_out"][0][:, 0]
            logits, _ = model.forward(c, pad, conf, tokens[:, :-1])
        enc = enc_out.double().numpy()
        lps.append(torch.log_softmax(logits[0].transpose(0, 1).double(), -1).numpy())
        lls.append(float(cf.score_sequence_batch(model, alphabet, [coords.astype(np.float64 if dtype == torch.float64 else np.float32)], [seq])[0]))
    return enc, lps, np.array(lls, dtype=np.float64)


def main():
    import pandas as pd
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cf = reference()
    out = {}

    # the reference's key names and shapes: the toy model, and the released widths on the meta device (no weights allocated)
    import argparse
    esm = cf.esm
    alphabet = esm.data.Alphabet.from_architecture(K.TOY_ARGS["arch"])
    assert list(alphabet.all_toks) == E.ALL_TOKS
    keys = {}
    for name, args in (("toy", K.TOY_ARGS), ("released", K.RELEASED_ARGS)):
        with torch.device("meta"):
            m = esm.inverse_folding.gvp_transformer.GVPTransformerModel(argparse.Namespace(**args), alphabet)
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    # the option strings of the reference script's parser (it is built inside main(), so they are read from the file's text)
    import re
    keys["cli_flags"] = re.findall(r"add_argument\(\s*['\"](--[^'\"]+)['\"]", open(cf.__file__).read())
    with open(os.path.join(HERE, "esmif1_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)

    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        torch.set_default_dtype(dtype)
        model, alphabet = build_model(cf, dtype)
        for name in K.CASES:
            coords, seqs = K.case(name)
            enc, lps, lls = run_case(cf, model, alphabet, coords, seqs, dtype)
            out[f"{name}_enc{tag}"] = enc
            for i, lp in enumerate(lps):
                out[f"{name}_lp{tag}_{i}"] = lp
            out[f"{name}_ll{tag}"] = lls
            print(name, tag, enc.shape, lls, flush=True)
    torch.set_default_dtype(torch.float32)
    np.savez_compressed(os.path.join(HERE, "golden_esmif1.npz"), **out)

    # the toy assay through score_singlechain_backbone_batch, load_coords fed from the repository's reader
    fname, L, seed, nan_ca, first = K.TOY_PDB
    os.makedirs(os.path.join(HERE, "ESMIF1_structures"), exist_ok=True)
    wt = K.sequence_of(seed, L)
    with open(os.path.join(HERE, "ESMIF1_structures", fname), "w") as f:
        f.write(K.pdb_text(wt, K.backbone(seed, L, nan_ca), first))
    rng = np.random.default_rng(13)
    mutants, seqs = [], []
    for p in rng.choice(L, 10, replace=False):
        to = rng.choice([a for a in K.AA if a != wt[p]])
        mutants.append(f"{wt[p]}{p + 1}{to}")
        seqs.append(wt[:p] + to + wt[p + 1:])
    mutants.append("WT_like")                                  # the `mutant` column is a label: nothing parses it
    seqs.append(wt)
    mutants.append("shorter")                                  # a sequence whose length differs from the structure's
    seqs.append(wt[:-3])
    pd.DataFrame({"mutant": mutants, "mutated_sequence": seqs, "DMS_score": rng.standard_normal(len(seqs)).round(4)}).to_csv(
        os.path.join(HERE, "TOY_ESMIF1.csv"), index=False)
    pd.DataFrame({"DMS_id": ["TOY_ESMIF1"], "DMS_filename": ["TOY_ESMIF1.csv"], "target_seq": [wt], "pdb_file": [fname]}).to_csv(
        os.path.join(HERE, "TOY_ESMIF1_REFERENCE.csv"), index=False)
    model, alphabet = build_model(cf, torch.float32)
    cf.esm.inverse_folding.util.load_coords = lambda fpath, chain: E.read_backbone(fpath, chain)
    cf.score_singlechain_backbone_batch(model, alphabet, pdb_file=os.path.join(HERE, "ESMIF1_structures", fname), chain="A",
                                        mutation_file=os.path.join(HERE, "TOY_ESMIF1.csv"),
                                        output_filepath=os.path.join(HERE, "TOY_ESMIF1_reference_scores.csv"), batch_size=1, nogpu=True)
    print(open(os.path.join(HERE, "TOY_ESMIF1_reference_scores.csv")).read())


if __name__ == "__main__":
    main()
