"""CARP assay scoring on MI355X: what ProteinGym's ``CARP_600K``, ``CARP_38M``, ``CARP_76M`` and ``CARP_640M`` rows read.

The flags are proteingym/baselines/carp_mif/compute_fitness.py's.  The assay is row --DMS_index of --DMS_reference_file_path, its CSV is
read from --DMS_data_folder, and ``<output_scores_folder>/<model_name>/<DMS_id>.csv`` gets the columns mutant, <model_name>_score,
DMS_score; one ``DMS_id,spearman`` line is appended to --performance_file, whose header is written once.
--fitness_computation_mode masked_marginals (the default): one forward of the wild type per mutated position with that token masked,
a mutant scores the mean over its substitutions of lp[i, mt] - lp[i, wt].  pseudo_likelihood: one unmasked forward per mutated
sequence, the mean over its tokens of log p(x_t); with --indel_mode the ``mutant`` column is the sequence itself.
--model_name is a checkpoint name resolved as ``<model_path>/<name>.pt`` or a path ending in .pt; nothing is downloaded.  MIF and
MIF-ST are refused.  --structure_data_folder is accepted and ignored.  Additive flags: --device, --precision, --max_rows.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import _lib, carp


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="CARP scoring (HIP, MI355X)")
    p.add_argument("--model_name", type=str, required=True, help="checkpoint name (resolved under --model_path) or a path ending in .pt")
    p.add_argument("--model_path", type=str, default=None, help="folder holding the checkpoints")
    p.add_argument("--DMS_reference_file_path", type=str, required=True, help="reference CSV listing the assays")
    p.add_argument("--DMS_data_folder", type=str, required=True, help="folder holding the assay CSVs")
    p.add_argument("--structure_data_folder", type=str, default="", help="accepted; CARP reads no structure")
    p.add_argument("--DMS_index", type=int, required=True)
    p.add_argument("--output_scores_folder", type=str, required=True)
    p.add_argument("--indel_mode", action="store_true", help="the mutant column holds the sequences themselves")
    p.add_argument("--fitness_computation_mode", type=str, default="masked_marginals", choices=["masked_marginals", "pseudo_likelihood"])
    p.add_argument("--performance_file", type=str, default="CARP_performance.csv")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--precision", type=str, default="f16x3", choices=["f16x3", "fp32"])
    p.add_argument("--max_rows", type=int, default=0, help="rows per device chunk (0 = library default)")
    return p


class Scorer:
    """The model of the run; a forward that leaves the fp16 range (PGMI_EOVERFLOW) is repeated on an fp32 model, built once."""

    def __init__(self, path: str, device: int, precision: str, max_rows: int):
        self.args = (path, device, max_rows)
        self.model = carp.from_pretrained(path, device=device, precision=precision, max_rows=max_rows)
        self.fp32 = None

    def run(self, fn, *a) -> np.ndarray:
        try:
            return fn(self.model, *a)
        except _lib.PgmiError as e:
            if e.code != _lib.EOVERFLOW:
                raise
        print("[proteingym_amd] an activation left the fp16 range: scoring this assay in precision fp32", file=sys.stderr)
        if self.fp32 is None:
            path, device, max_rows = self.args
            self.fp32 = carp.from_pretrained(path, device=device, precision="fp32", max_rows=max_rows)
        return fn(self.fp32, *a)

    def close(self):
        for m in (self.model, self.fp32):
            if m is not None:
                m.close()


def spearman(a, b) -> float:
    import pandas as pd
    return float(pd.Series(np.asarray(a, dtype=np.float64)).corr(pd.Series(np.asarray(b, dtype=np.float64)), method="spearman"))


def main(argv=None):
    import pandas as pd
    args = parser().parse_args(argv)
    if "mif" in os.path.basename(args.model_name).lower():
        raise _lib.PgmiError(f"{args.model_name!r}: MIF and MIF-ST need the structure GNN and are not supported; CARP checkpoints only")
    if args.indel_mode and args.fitness_computation_mode != "pseudo_likelihood":
        raise _lib.PgmiError("--indel_mode needs --fitness_computation_mode pseudo_likelihood (masked marginals score substitutions)")
    path = carp.resolve_checkpoint(args.model_name, args.model_path)
    mapping = pd.read_csv(args.DMS_reference_file_path)
    DMS_id = mapping["DMS_id"][args.DMS_index]
    # the checkpoint's name, as the reference uses it (config.json: CARP/carp_640M, carp_640M_score); a path ending in .pt gives its file stem
    label = os.path.basename(args.model_name)[:-3] if args.model_name.endswith(".pt") else carp.MODEL_NAMES.get(args.model_name, args.model_name)
    folder = args.output_scores_folder + os.sep + label
    os.makedirs(folder, exist_ok=True)
    scoring_filename = folder + os.sep + str(DMS_id) + ".csv"
    print(f"Computing scores for: {DMS_id} with model: {args.model_name}")
    row = mapping[mapping["DMS_id"] == DMS_id]
    target_seq = row["target_seq"].values[0].upper()
    DMS_data = pd.read_csv(args.DMS_data_folder + os.sep + row["DMS_filename"].values[0], low_memory=False)
    scorer = Scorer(path, args.device, args.precision, args.max_rows)
    try:
        if args.fitness_computation_mode == "masked_marginals":
            scores = scorer.run(carp.masked_marginal_scores, target_seq, list(DMS_data["mutant"]))
        else:
            seqs = list(DMS_data["mutant"]) if args.indel_mode else [carp.get_mutated_sequence(target_seq, m) for m in DMS_data["mutant"]]
            scores = scorer.run(carp.pseudo_likelihood_scores, seqs)
    finally:
        scorer.close()
    col = label + "_score"
    DMS_data[col] = scores
    DMS_data[["mutant", col, "DMS_score"]].to_csv(scoring_filename, index=False)
    rho = spearman(DMS_data[col], DMS_data["DMS_score"])
    if not os.path.exists(args.performance_file) or os.stat(args.performance_file).st_size == 0:
        with open(args.performance_file, "w") as f:
            f.write("DMS_id,spearman\n")
    with open(args.performance_file, "a") as f:
        f.write(",".join([str(DMS_id), str(rho)]) + "\n")
    return scoring_filename


if __name__ == "__main__":
    main()
