"""Drop-in for ``proteingym/baselines/esm/compute_fitness_esm_if1.py`` on MI355X.

Same flags, mixed spellings included, and the same file: ``<output_scores_folder>/<DMS_id>.csv`` with the header ``mutant,esmif1_ll`` and
one row per line of the assay's ``mutant`` / ``mutated_sequence`` columns -- the mean log-likelihood of the mutated sequence given the
backbone of ``--chain`` in ``<structure_folder>/<pdb_file>``, written as str() of a numpy float64 as the reference writes it.

The reference encodes the backbone again for every batch of mutants; here it is encoded once per assay and a mutant costs the decoder
only, so --batch_size is accepted and has no effect on the score.  --multichain-backbone / --singlechain-backbone are
parsed and ignored, as in the reference (its main() never reads the flag).  --nogpu is refused: the decoder has no CPU path.
Additive flags: --device, --max_batch, --max_rows."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import esmif1


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Score sequences based on a given structure (ESM-IF1; HIP, MI355X).")
    p.add_argument("--DMS_reference_file_path", type=str, help="path to DMS reference file")
    p.add_argument("--DMS_data_folder", type=str, help="path to folder containing DMS data")
    p.add_argument("--structure_folder", type=str, help="folder containing pdb files for each DMS")
    p.add_argument("--DMS_index", type=int, help="index of DMS in DMS reference file")
    p.add_argument("--model_location", type=str, help="path to model")
    p.add_argument("--batch_size", type=int, default=1, help="accepted; no effect (the backbone is encoded once, mutants are packed)")
    p.add_argument("--output_scores_folder", type=str, help="path to folder where scores will be saved")
    p.add_argument("--chain", type=str, help="chain id for the chain of interest", default="A")
    p.set_defaults(multichain_backbone=False)
    p.add_argument("--multichain-backbone", action="store_true", help="parsed and ignored, as in the reference")
    p.add_argument("--singlechain-backbone", dest="multichain_backbone", action="store_false",
                   help="use the backbone of only target chain in the input for conditioning")
    p.add_argument("--nogpu", action="store_true", help="refused: the decoder runs in HIP only")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_batch", type=int, default=4096, help="mutants per call into the library")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows of the decoder (0: the library's default)")
    return p


def main(argv=None, model=None) -> str:
    """Scores one assay and returns the path of the CSV.  ``model``: an esmif1.EsmIf1Model to use instead of --model_location (tests)."""
    args = parser().parse_args(argv)
    if args.nogpu:
        raise SystemExit("--nogpu: the ESM-IF1 decoder runs on the GPU only (libpgmi has no CPU path)")
    mapping = pd.read_csv(args.DMS_reference_file_path)
    row = mapping.iloc[args.DMS_index]
    out_path = args.output_scores_folder + os.sep + row["DMS_id"] + ".csv"
    os.makedirs(args.output_scores_folder, exist_ok=True)
    coords, _ = esmif1.read_backbone(args.structure_folder + os.sep + row["pdb_file"], args.chain)
    df = pd.read_csv(args.DMS_data_folder + os.sep + row["DMS_filename"])
    names, seqs = df["mutant"].tolist(), df["mutated_sequence"].tolist()
    own = model is None
    if own:
        cfg, sd = esmif1.load_checkpoint(args.model_location)
        model = esmif1.EsmIf1Model(cfg, sd, device=args.device, max_rows=args.max_rows, max_memory=len(coords) + 2)
    try:
        model.set_structure(coords)
        scores = model.score(seqs, max_batch=args.max_batch)
    finally:
        if own:
            model.close()
    with open(out_path, "w") as f:
        f.write("mutant,esmif1_ll\n")
        for name, ll in zip(names, scores):
            f.write(name + "," + str(np.float64(ll)) + "\n")
    return out_path


if __name__ == "__main__":
    main(sys.argv[1:])
