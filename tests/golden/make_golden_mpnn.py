"""Writes the ProteinMPNN fixtures under tests/golden/ProteinMPNN_toy/ and records TOY_PMPNN_REFERENCE.csv from the UNMODIFIED
reference (proteingym/baselines/protein_mpnn/compute_fitness.py, its own main() on the CPU through tests/mpnn_reference.py):

    toy.pdb                      synthetic two-chain backbone, L = 70: chain A residues 1 .. 38 with number 17 absent (one masked X),
                                 chain B residues 5 .. 36 with residue 20 lacking its O (masked, letter kept); side-chain CB records,
                                 one insertion code and one HETATM MSE are there for the parser
    TOY_PMPNN_DMS.csv            12 rows: mutant, mutated_sequence (70 letters; the sequence at the absent number is X)
    TOY_PMPNN_MAPPING.csv        DMS_id, DMS_filename, pdb_file
    TOY_PMPNN_RANDN.npy          float32 [12, 70]: the normals the reference drew for the decoding orders, in row order
    TOY_PMPNN_REFERENCE.csv      the reference's own output file: mutant, mutated_sequence, pmpnn_ll

    python tests/golden/make_golden_mpnn.py

The checkpoint is proteingym_amd.mpnn.random_state_dict(7) with num_edges 48, written to a temporary directory: no checkpoint is
committed (6.6 MB); the tests rebuild it from the same seed."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from proteingym_amd import mpnn  # noqa: E402
import mpnn_cases as mc  # noqa: E402
import mpnn_reference as mr  # noqa: E402

OUT = os.path.join(HERE, "ProteinMPNN_toy")
AA3 = dict(zip("ARNDCQEGHILKMFPSTWYV", mpnn._AA3))
SEED, NUM_EDGES = 7, 48


def atom_line(serial, atom, res3, chain, num, icode, xyz, het=False):
    return (f"{'HETATM' if het else 'ATOM  '}{serial:5d} {atom:<4s} {res3:>3s} {chain}{num:4d}{icode:1s}   "
            f"{xyz[0]:8.3f}{xyz[1]:8.3f}{xyz[2]:8.3f}  1.00  0.00           {atom[0]:>1s}")


def write_pdb(path):
    rng = np.random.default_rng(11)
    X = mc.backbone(71, 21)              # 71 walk positions: one is the absent residue number
    letters = rng.choice(list("ARNDCQEGHILKMFPSTWYV"), size=71)
    lines, serial, w = [], 1, 0
    for chain, nums in (("B", list(range(5, 37))), ("A", list(range(1, 39)))):        # B first in the file: chains are sorted
        for num in nums:
            pos = w
            w += 1
            if chain == "A" and num == 17:
                continue                                                             # absent residue number
            icode = "A" if (chain == "B" and num == 30) else " "                     # an insertion code is a residue of its own
            res3 = AA3[letters[pos]]
            het = chain == "A" and num == 9
            if het:
                res3 = "MSE"
            for a, name in enumerate(("N", "CA", "C", "O")):
                if chain == "B" and num == 20 and name == "O":
                    continue
                lines.append(atom_line(serial, name, res3, chain, num, icode, X[pos, a], het))
                serial += 1
            lines.append(atom_line(serial, "CB", res3, chain, num, icode, X[pos, 1] + 1.5, het))
            serial += 1
            if num == 12:                                                            # a repeated record: the first one wins
                lines.append(atom_line(serial, "CA", res3, chain, num, icode, X[pos, 1] + 9.0, het))
                serial += 1
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\nEND\n")


def main():
    import pandas as pd
    os.makedirs(OUT, exist_ok=True)
    pdb = os.path.join(OUT, "toy.pdb")
    write_pdb(pdb)
    feat = mpnn.featurize(mpnn.parse_pdb(pdb))
    wt, L = feat["seq"], len(feat["seq"])
    assert L == 70 and feat["mask"].sum() == 68, (L, feat["mask"].sum())
    assert mc.neighbour_gap_ok(dict(X=feat["X"], mask=feat["mask"]), NUM_EDGES)
    rng = np.random.default_rng(5)
    rows = [("wt", wt)]
    for r in range(11):
        s = list(wt)
        names = []
        for i in rng.choice([i for i in range(L) if wt[i] != "X"], size=1 + r % 2, replace=False):
            new = rng.choice([a for a in "ACDEFGHIKLMNPQRSTVWY" if a != wt[i]])
            names.append(f"{wt[i]}{i + 1}{new}")
            s[i] = new
        rows.append((":".join(names), "".join(s)))
    pd.DataFrame(rows, columns=["mutant", "mutated_sequence"]).to_csv(os.path.join(OUT, "TOY_PMPNN_DMS.csv"), index=False)
    pd.DataFrame([{"DMS_id": "TOY_PMPNN", "DMS_filename": "TOY_PMPNN_DMS.csv", "pdb_file": "toy.pdb"}]).to_csv(
        os.path.join(OUT, "TOY_PMPNN_MAPPING.csv"), index=False)
    tmp = tempfile.mkdtemp()
    try:
        ck = os.path.join(tmp, "toy.pt")
        mpnn.save_checkpoint(ck, mpnn.random_state_dict(SEED), NUM_EDGES)
        drawn = []
        mr.run_script(["--DMS_reference_file_path", os.path.join(OUT, "TOY_PMPNN_MAPPING.csv"), "--DMS_data_folder", OUT,
                       "--structure_folder", OUT, "--DMS_index", "0", "--checkpoint", ck, "--output_scores_folder", tmp, "--seed", "3",
                       "--suppress_print", "1"], record=drawn)
        drawn = [d for d in drawn if d.shape == (1, L)]
        assert len(drawn) == len(rows), len(drawn)
        np.save(os.path.join(OUT, "TOY_PMPNN_RANDN.npy"), np.concatenate(drawn, 0).astype(np.float32))
        shutil.copy(os.path.join(tmp, "TOY_PMPNN.csv"), os.path.join(OUT, "TOY_PMPNN_REFERENCE.csv"))
    finally:
        shutil.rmtree(tmp)
    print(open(os.path.join(OUT, "TOY_PMPNN_REFERENCE.csv")).read())


if __name__ == "__main__":
    main()
