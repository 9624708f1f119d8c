"""Drop-in for ``proteingym/baselines/mulan/compute_fitness.py`` on MI355X.

Same flags and the same assay loop (:129-259): the assay is row --DMS_index of --DMS_reference_file_path, its ``pdb_file`` / ``pdb_range``
cells are split on ``|`` into structure chunks (ranges 1-indexed, inclusive), a mutant belongs to the chunk that holds the position of
its FIRST sub-mutation, every chunk is scored on its own dataset sequence and angle rows, and the per-chunk score arrays are
concatenated in chunk order and assigned to the rows POSITIONALLY, as in the reference.  The input tokens are the chunk's DATASET
sequence -- the residues of the structure file, MSE as X -- not ``target_seq``; a mutant's letters only pick the columns that are read.
Output: ``<output_scores_folder>/<DMS_id>.csv`` with the columns mutant, MULAN_score, DMS_score.  Unlike SaProt's script an existing
output file is NOT recomputed (:209-211).  ``POLG_HCVJF_Qi_2014``'s first range start is shifted by one (:242-245).

Angle rows: the reference's cached dataset folder (--output_dataset_folder with test_names.json ...) when it exists, else the
structure file through proteingym_amd.mulan.structure_rows (and, with --use_foldseek, Foldseek run as the SaProt script runs it).  The
folder is read, never written.  The model is a local checkpoint directory; nothing is downloaded (--hf_cache_folder is accepted and
unused).

Divergences, all deliberate: --indel_mode exits with 2 (the reference's own path cannot parse an indel); a dataset sequence whose
length differs from its angle rows is a ValueError; a sub-mutation outside its chunk is a ValueError naming the mutant (the reference
wraps a negative index); a 16-bit forward that leaves the fp16 range is re-run on an fp32 model; any encoder depth is taken (the
reference's auto_detect_base_tokenizer knows 6 and 12).  Additive flags: --device, --precision, --max_rows.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import _lib, mulan, saprot


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="MULAN scoring (HIP, MI355X)")
    p.add_argument("--MULAN_model_name_or_path", default="", type=str, help="Path to a local MULAN checkpoint directory")
    p.add_argument("--DMS_reference_file_path", default="", type=str, help="Path of the DMS reference file")
    p.add_argument("--DMS_data_folder", default="", type=str, help="Path of DMS folder")
    p.add_argument("--structure_data_folder", default="", type=str, help="Path of structure folder")
    p.add_argument("--DMS_index", type=int, help="Index of the assay in the reference file")
    p.add_argument("--use_foldseek", action="store_true", help="Whether the model uses foldseek sequences")
    p.add_argument("--foldseek_path", default="./bin/foldseek", type=str, help="Path of foldseek binary file")
    p.add_argument("--output_scores_folder", default=None, type=str, help="Name of folder to write model scores to")
    p.add_argument("--output_dataset_folder", default="", type=str, help="Folder of the preprocessed MULAN dataset (read if present)")
    p.add_argument("--hf_cache_folder", default="", type=str, help="accepted for compatibility; nothing is downloaded")
    p.add_argument("--indel_mode", action="store_true", help="Whether to score sequences with insertions and deletions (not supported)")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--precision", choices=sorted(_lib.PRECISIONS), default="f16x3", help="GEMM operand precision")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")
    return p


class Scorer:
    """The model of the run; a forward that leaves the 16-bit range (PGMI_EOVERFLOW) is repeated on an fp32 model, built once."""

    def __init__(self, path: str, use_foldseek: bool, device: int, precision: str, max_rows: int):
        self.args = (path, use_foldseek, device, max_rows)
        self.model = mulan.from_pretrained(path, use_foldseek, device=device, precision=precision, max_rows=max_rows)
        self.fp32 = None

    def score_chunk(self, *a) -> np.ndarray:
        try:
            return self.model.score_chunk(*a)
        except _lib.PgmiError as e:
            if e.code != _lib.EOVERFLOW:
                raise
        print("[proteingym_amd] an activation left the fp16 range: scoring this chunk in precision fp32", file=sys.stderr)
        if self.fp32 is None:
            path, use_foldseek, device, max_rows = self.args
            self.fp32 = mulan.from_pretrained(path, use_foldseek, device=device, precision="fp32", max_rows=max_rows)
        return self.fp32.score_chunk(*a)

    def close(self):
        for m in (self.model, self.fp32):
            if m is not None:
                m.close()


def chunk_inputs(dataset, structure_folder: str, pdb_filename: str, use_foldseek: bool, foldseek_path: str):
    """(dataset sequence, rows [L][11]) of one chunk: the cached dataset's entry named like the file (:231), else the file itself."""
    if dataset is not None:
        name = pdb_filename[:-4]
        if name not in dataset:
            raise IndexError(f"{name}: not in the dataset folder's names")         # the reference's dataset_id_index[0]
        return dataset[name]
    path = structure_folder + os.sep + pdb_filename
    seq, rows = mulan.structure_rows(path)
    if use_foldseek:
        struc = saprot.structure_sequence(foldseek_path, path)
        if len(struc) != len(seq):
            raise ValueError(f"{pdb_filename}: Foldseek string has {len(struc)} letters, the structure's sequence {len(seq)}")
        seq = "".join(a + s for a, s in zip(seq, struc))
    return seq, rows


def score_assay(scorer, dataset, args, DMS_id: str, target_seq: str, pdb_files, pdb_ranges, mutants) -> np.ndarray:
    """compute_fitness.py:229-255: the concatenation of the chunks' score arrays."""
    first_pos = np.array([int(str(m).split(":")[0][1:-1]) for m in mutants], dtype=np.int64)
    model_scores = []
    for pdb_filename, pdb_range in zip(pdb_files, pdb_ranges):
        lo, hi = (int(x) for x in pdb_range.split("-"))
        if DMS_id == "POLG_HCVJF_Qi_2014":                   # the shift between the pdb sequence and the target sequence (:242-245)
            lo += 1
        seq, rows = chunk_inputs(dataset, args.structure_data_folder, pdb_filename, args.use_foldseek, args.foldseek_path)
        n_res = len(seq) // 2 if args.use_foldseek else len(seq)
        if n_res != len(rows):
            raise ValueError(f"{pdb_filename}: the dataset sequence has {n_res} residues, its angle rows {len(rows)}")
        idx = np.flatnonzero((first_pos >= lo) & (first_pos <= hi))
        if idx.size == 0:
            model_scores.append(np.zeros(0))
            continue
        parsed = mulan.parse_chunk([mutants[i] for i in idx], target_seq, lo, n_res, args.use_foldseek)
        angles, plddt = mulan.chunk_features(rows)
        model_scores.append(scorer.score_chunk(mulan.tokenize(seq, args.use_foldseek), angles, plddt, *parsed))
    return np.concatenate(model_scores) if model_scores else np.zeros(0)


def main(argv=None):
    args = parser().parse_args(argv)
    if args.indel_mode:
        print("--indel_mode is not supported: MULAN's scoring rule reads substitutions (A123B) only", file=sys.stderr)
        return 2
    if args.DMS_index is None or not args.output_scores_folder:
        print("--DMS_index and --output_scores_folder are required", file=sys.stderr)
        return 2
    mapping = pd.read_csv(args.DMS_reference_file_path)
    DMS_id = mapping["DMS_id"][args.DMS_index]
    row = mapping[mapping["DMS_id"] == DMS_id]
    scoring_filename = args.output_scores_folder + os.sep + DMS_id + ".csv"
    if os.path.exists(scoring_filename):
        print("Scores already computed for: {}".format(DMS_id))
        return 0
    print("Computing scores for: {}, {} with MULAN: {}".format(args.DMS_index, DMS_id, args.MULAN_model_name_or_path))
    target_seq = row["target_seq"].values[0].upper()
    DMS_data = pd.read_csv(args.DMS_data_folder + os.sep + row["DMS_filename"].values[0], low_memory=False)
    mutants = DMS_data["mutant"].tolist()
    # get_mutated_sequence's assertions (wild-type letter, target letter among the 20) over the whole column, before any forward
    mulan.parse_chunk(mutants, target_seq, 1, len(target_seq), args.use_foldseek)
    pdb_files, pdb_ranges = row["pdb_file"].values[0].split("|"), str(row["pdb_range"].values[0]).split("|")
    dataset = mulan.load_dataset_folder(args.output_dataset_folder, args.use_foldseek)
    scorer = Scorer(args.MULAN_model_name_or_path, args.use_foldseek, args.device, args.precision, args.max_rows)
    try:
        scores = score_assay(scorer, dataset, args, DMS_id, target_seq, pdb_files, pdb_ranges, mutants)
    finally:
        scorer.close()
    if len(scores) != len(DMS_data):                       # pandas' own error when a row falls in no chunk
        raise ValueError(f"Length of values ({len(scores)}) does not match length of index ({len(DMS_data)})")
    DMS_data["MULAN_score"] = scores
    os.makedirs(args.output_scores_folder, exist_ok=True)
    DMS_data[["mutant", "MULAN_score", "DMS_score"]].to_csv(scoring_filename, index=False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
