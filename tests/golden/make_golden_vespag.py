"""Writes tests/golden/VespaG_toy: the inputs of the CLI tests in tests/test_gpu_vespag.py.  Everything is seeded and made here; nothing
comes from a released checkpoint or a ProteinGym file.

    python tests/golden/make_golden_vespag.py

  state_dict_v2.pt     a seeded FNN([256], 128, 20) head (proteingym_amd.vespag.random_state_dict(**vespag_ref.TOY_HEAD))
  proteins.fasta       two proteins; TOY_B holds a U (tokenised as X, its row left unmasked)
  mutations.csv        a mutation file with a header line: single and ':'-joined mutants of both proteins
  reference.csv        a two-assay DMS reference file (DMS_id, DMS_filename, target_seq)
  DMS/TOY_A.csv, DMS/TOY_B.csv   mutant, DMS_score; TOY_B has multi-mutants
The small ESM2 the tests embed with is too large to commit; they rebuild it from its seed (vespag_ref.toy_esm).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import vespag_ref as R  # noqa: E402
from proteingym_amd import vespag  # noqa: E402

AA = "ACDEFGHIKLMNPQRSTVWY"


def main():
    out = os.path.join(HERE, "VespaG_toy")
    os.makedirs(os.path.join(out, "DMS"), exist_ok=True)
    rng = np.random.default_rng(20261021)
    torch.save({k: torch.from_numpy(v) for k, v in vespag.random_state_dict(**R.TOY_HEAD).items()}, os.path.join(out, "state_dict_v2.pt"))
    seqs = {"TOY_A": "".join(rng.choice(list(AA), 23)), "TOY_B": "".join(rng.choice(list(AA), 31))}
    seqs["TOY_B"] = seqs["TOY_B"][:11] + "U" + seqs["TOY_B"][12:]
    with open(os.path.join(out, "proteins.fasta"), "w") as f:
        for k, s in seqs.items():
            f.write(f">{k} seeded toy protein\n{s[:20]}\n{s[20:]}\n")

    def sav(s):
        i = int(rng.integers(len(s)))
        return f"{s[i]}{i + 1}{rng.choice([a for a in AA if a != s[i]])}"

    def mutants(s, n, multi):
        out = []
        for j in range(n):
            k = 1 + (int(rng.integers(1, 4)) if multi and j % 2 else 0)
            out.append(":".join(sav(s) for _ in range(k)))
        return list(dict.fromkeys(out))
    with open(os.path.join(out, "mutations.csv"), "w") as f:
        f.write("protein_id,mutation\n")
        for k, s in seqs.items():
            for m in mutants(s, 12, True):
                f.write(f"{k},{m}\n")
        f.write(f"TOY_A,{seqs['TOY_A'][0]}1{seqs['TOY_A'][0]}\n")             # to_aa == wild type
    with open(os.path.join(out, "reference.csv"), "w") as f:
        f.write("DMS_index,DMS_id,DMS_filename,target_seq\n")
        for i, (k, s) in enumerate(seqs.items()):
            f.write(f"{i},{k},{k}.csv,{s}\n")
    for k, s in seqs.items():
        with open(os.path.join(out, "DMS", f"{k}.csv"), "w") as f:
            f.write("mutant,DMS_score\n")
            for m in mutants(s, 30, k == "TOY_B"):
                f.write(f"{m},{rng.standard_normal():.4f}\n")


if __name__ == "__main__":
    main()
