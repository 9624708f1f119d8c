"""Records tests/golden/ProtSSN_toy/: a toy structure (two chains, one water record, one residue without C), a toy assay with ':'
mutants, ';' mutants and a wt row, the three normalisation files' pos_std / edge_attr_mean / edge_attr_std as one .npz, and the
float64 scores of tests/protssn_ref.py on them.

    python tests/golden/make_golden_protssn.py --norm_dir <ProteinGym>/proteingym/baselines/protssn/norm

torch_geometric and Bio are not installed, so the expected values come from the float64 restatement (tests/protssn_ref.py: the unsplit
first Linear on the concatenation, index_add_ over edge_index[1]) fed by a float64 HF EsmModel that holds the toy's seeded ESM2
weights, not from the library; DESIGN.md 4.6q lists what is read from the libraries' documented behaviour.  No test imports this file;
only the files it writes are committed."""
import argparse
import os
import sys

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import protssn_ref as R  # noqa: E402
from proteingym_amd import protssn, synthetic  # noqa: E402

OUT = os.path.join(HERE, "ProtSSN_toy")
ONE_TO_THREE = {v: k for k, v in protssn.THREE_TO_ONE.items()}
SEQ_A, SEQ_B = "MKVLAAGIVRHDESTNQCGPAVIFY", "WLMKRHDESTNQCGP"          # 25 + 15 residues


def atom_line(serial, name, resname, chain, resseq, xyz, record="ATOM  "):
    return (f"{record}{serial:5d} {name:<4s} {resname:>3s} {chain}{resseq:4d}    {xyz[0]:8.3f}{xyz[1]:8.3f}{xyz[2]:8.3f}"
            f"{1.0:6.2f}{50.0:6.2f}          {name[0]:>2s}")


def write_pdb(path):
    ca = R.serpentine(len(SEQ_A) + len(SEQ_B) + 1, seed=4)
    n, ca, c = R.toy_backbone(ca, seed=5)
    lines, serial, i = ["HEADER    TOY STRUCTURE FOR PROTSSN"], 1, 0
    for chain, seq in (("A", SEQ_A), ("B", SEQ_B)):
        for r, aa in enumerate(seq, start=1):
            for name, xyz in (("N", n[i]), ("CA", ca[i]), ("C", c[i])):
                lines.append(atom_line(serial, name, ONE_TO_THREE[aa], chain, r, xyz))
                serial += 1
            i += 1
            if chain == "A" and r == 12:            # a residue without C between A12 and A13: dropped, numbering continues
                for name, xyz in (("N", n[-1]), ("CA", ca[-1])):
                    lines.append(atom_line(serial, name, "GLY", "A", 112, xyz))
                    serial += 1
        lines.append("TER")
    lines.append(atom_line(serial, "O", "HOH", "A", 301, ca[3] + 3.0, record="HETATM"))
    lines.append("END")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--norm_dir", required=True)
    args = ap.parse_args()
    folder = os.path.join(OUT, "DATASET", R.TOY_NAME)
    os.makedirs(folder, exist_ok=True)
    norms = {k: protssn.load_norm(k, norm_dir=args.norm_dir) for k in protssn.KS}
    np.savez(os.path.join(OUT, "protssn_norm.npz"), **{f"k{k}_{n}": a for k, d in norms.items() for n, a in d.items()})
    pdb = os.path.join(folder, R.TOY_NAME + ".pdb")
    write_pdb(pdb)
    n, ca, c, seq = protssn.read_pdb(pdb)
    assert seq == SEQ_A + SEQ_B, seq
    s = lambda i, mt: f"{seq[i - 1]}{i}{mt}"
    mutants = [s(1, "A"), s(5, "G"), s(13, "W"), s(25, "C"), s(26, "A"), s(40, "K"), f"{s(2, 'R')}:{s(30, 'E')}",
               f"{s(7, 'P')}:{s(8, 'D')}:{s(39, 'Y')}", f"{s(3, 'I')};{s(17, 'F')}", f"{s(20, 'T')};{s(33, 'H')};{s(34, 'N')}", "wt", "WT"]
    rng = np.random.default_rng(9)
    df = pd.DataFrame({"mutant": mutants, "DMS_score": np.round(rng.standard_normal(len(mutants)), 4)})
    df.to_csv(os.path.join(folder, R.TOY_NAME + ".tsv"), sep="\t", index=False)
    cfg, blob = R.toy_esm()
    esm = R.fair_to_hf(synthetic.blob_to_arrays(cfg, blob), cfg)
    rows = R.hf_residue_rows(esm, protssn.tokenize(seq))
    for name, k, h, seed in R.TOY_MODELS:
        pos, centre, nb, ea = protssn.build_graph(n, ca, c, k, norms[k])
        lp, _ = R.forward(R.toy_state_dict(h, seed), rows, pos, centre, nb, ea)
        df[f"ProtSSN_{name}"] = [R.label_row(m, seq, lp.numpy()) for m in mutants]
    df["ProtSSN_ensemble"] = df[[f"ProtSSN_{m[0]}" for m in R.TOY_MODELS]].mean(axis=1)
    df.to_csv(os.path.join(OUT, "reference.csv"), index=False, float_format="%.10g")
    print(df)


if __name__ == "__main__":
    main()
