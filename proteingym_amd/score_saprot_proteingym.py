"""Drop-in for ``proteingym/baselines/saprot/compute_fitness.py`` on MI355X.

Same flags and the same assay loop (:98-162): the assay is row --DMS_index of --DMS_reference_file_path, its ``pdb_file`` / ``pdb_range``
cells are split on ``|`` into structure chunks (ranges 1-indexed, inclusive), a mutant belongs to the chunk that holds the position of
its FIRST sub-mutation, every chunk is scored on its own structure string, and the per-chunk score arrays are concatenated in chunk
order and assigned to the rows POSITIONALLY -- rows interleaved between chunks get each other's scores, as in the reference, and a
row that falls in no chunk is the reference's length-mismatch ValueError.  Output: ``<output_scores_folder>/<DMS_id>.csv`` with the
columns mutant, SaProt_score, DMS_score (an existing file is reported and overwritten).  The model is a local Hugging Face checkpoint
directory; nothing is downloaded.  Foldseek is the user's executable, run with the reference's command line.

Divergences, all deliberate: --indel_mode exits with 2 (the reference's own path cannot parse an indel); a structure string whose
length differs from its chunk's sequence is a ValueError (the reference's zip truncates silently); a sub-mutation of a multi-mutant
outside its chunk is a ValueError naming the mutant (the reference wraps a negative index); a 16-bit forward that leaves the fp16
range is re-run on an fp32 model.  Additive flags: --device, --precision, --max_rows.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import _lib, saprot


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="SaProt scoring (HIP, MI355X)")
    p.add_argument("--foldseek_bin", default="", type=str, help="Path to foldseek binary file")
    p.add_argument("--SaProt_model_name_or_path", default="", type=str, help="Path to a local SaProt checkpoint directory")
    p.add_argument("--DMS_reference_file_path", default="", type=str, help="Path of the DMS reference file")
    p.add_argument("--DMS_data_folder", default="", type=str, help="Path of DMS folder")
    p.add_argument("--structure_data_folder", default="", type=str, help="Path of structure folder")
    p.add_argument("--DMS_index", type=int, help="Index of the assay in the reference file")
    p.add_argument("--output_scores_folder", default=None, type=str, help="Name of folder to write model scores to")
    p.add_argument("--indel_mode", action="store_true", help="Whether to score sequences with insertions and deletions (not supported)")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--precision", choices=sorted(_lib.PRECISIONS), default="f16x3", help="GEMM operand precision")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")
    return p


class Scorer:
    """The model of the run; a forward that leaves the 16-bit range (PGMI_EOVERFLOW) is repeated on an fp32 model, built once."""

    def __init__(self, path: str, device: int, precision: str, max_rows: int):
        self.args = (path, device, max_rows)
        self.model = saprot.from_pretrained(path, device=device, precision=precision, max_rows=max_rows)
        self.fp32 = None

    def score_chunk(self, *a) -> np.ndarray:
        try:
            return self.model.score_chunk(*a)
        except _lib.PgmiError as e:
            if e.code != _lib.EOVERFLOW:
                raise
        print("[proteingym_amd] an activation left the fp16 range: scoring this chunk in precision fp32", file=sys.stderr)
        if self.fp32 is None:
            path, device, max_rows = self.args
            self.fp32 = saprot.from_pretrained(path, device=device, precision="fp32", max_rows=max_rows)
        return self.fp32.score_chunk(*a)

    def close(self):
        for m in (self.model, self.fp32):
            if m is not None:
                m.close()


def score_assay(scorer, foldseek_bin: str, structure_folder: str, target_seq: str, pdb_files, pdb_ranges, mutants) -> np.ndarray:
    """compute_fitness.py:142-158: the concatenation of the chunks' score arrays."""
    first_pos = np.array([int(str(m).split(":")[0][1:-1]) for m in mutants], dtype=np.int64)
    model_scores = []
    for pdb_filename, pdb_range in zip(pdb_files, pdb_ranges):
        lo, hi = (int(x) for x in pdb_range.split("-"))
        chunk_seq = target_seq[lo - 1:hi]
        rows = np.flatnonzero((first_pos >= lo) & (first_pos <= hi))
        struc = saprot.structure_sequence(foldseek_bin, structure_folder + os.sep + pdb_filename)
        if len(struc) != len(chunk_seq):
            raise ValueError(f"{pdb_filename}: structure string has {len(struc)} letters, its chunk {lo}-{hi} of the target sequence "
                             f"{len(chunk_seq)}")
        if rows.size == 0:
            model_scores.append(np.zeros(0))
            continue
        parsed = saprot.parse_chunk([mutants[i] for i in rows], target_seq, lo, len(chunk_seq))
        model_scores.append(scorer.score_chunk(saprot.tokenize(chunk_seq, struc), *parsed))
    return np.concatenate(model_scores) if model_scores else np.zeros(0)


def main(argv=None):
    args = parser().parse_args(argv)
    if args.indel_mode:
        print("--indel_mode is not supported: SaProt's scoring rule reads substitutions (A123B) only", file=sys.stderr)
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
    print("Computing scores for: {} with SaProt: {}".format(DMS_id, args.SaProt_model_name_or_path))
    target_seq = row["target_seq"].values[0].upper()
    DMS_data = pd.read_csv(args.DMS_data_folder + os.sep + row["DMS_filename"].values[0], low_memory=False)
    mutants = DMS_data["mutant"].tolist()
    # get_mutated_sequence's assertions (wild-type letter, target letter among the 20) over the whole column, before any forward
    saprot.parse_chunk(mutants, target_seq, 1, len(target_seq))
    pdb_files, pdb_ranges = row["pdb_file"].values[0].split("|"), str(row["pdb_range"].values[0]).split("|")
    scorer = Scorer(args.SaProt_model_name_or_path, args.device, args.precision, args.max_rows)
    try:
        scores = score_assay(scorer, args.foldseek_bin, args.structure_data_folder, target_seq, pdb_files, pdb_ranges, mutants)
    finally:
        scorer.close()
    if len(scores) != len(DMS_data):                       # pandas' own error when a row falls in no chunk
        raise ValueError(f"Length of values ({len(scores)}) does not match length of index ({len(DMS_data)})")
    DMS_data["SaProt_score"] = scores
    os.makedirs(args.output_scores_folder, exist_ok=True)
    DMS_data[["mutant", "SaProt_score", "DMS_score"]].to_csv(scoring_filename, index=False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
